#!/usr/bin/env python3
"""What the search statistics per training row (include/taflhip.h TAFL_EXAMPLES_SEARCH_STATS) cost on one MI355X, by
the protocol of tools/measure_eval_symmetry.py: 65 536 Copenhagen 11x11 lanes, S simulations per root, a free evaluator (constant
float32 priors and zero values resident in HBM).

(a), (b)  the library's share of a round of a recording guided self-play run (`--moves` moves per lane into an examples object with
          max_children = 64): the wall time of one whole run - tafl_gselfplay_begin, every tafl_gselfplay_step (each returns the waiting
          count, so each ends in a stream synchronise) - over its rounds.  Mode `off`: an examples object without the flag, nothing of
          the feature runs; mode `on`: with the flag, k_gselfplay_record_stats follows every round.
(c)       tafl_pool_ingest of the run's finalized examples with the pool's setting off and on, and tafl_examples_gather_stats at
          4 096 and 65 536 rows (device pointers), in microseconds between two events on the library's stream, with the bytes moved.

`--modes off,on` alternates inside one process, `--reps` times; `--lib` with `--modes off` runs another build of the library (the
parent commit's), binding what it exports.  Prints one JSON line per measurement and, with --out, appends them to that file;
`--summarise FILE` reads such a file and applies the rule: the off range of this build must overlap the parent's range or exceed its
upper end by no more than the parent's own spread (max - min), for the round and for the ingest."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(path):
    rows = [json.loads(x) for x in open(path) if x.strip()]
    out, ok = {}, True
    for what, key in (("round", "ms_per_round"), ("ingest", "ingest_us_min")):
        r = {}
        for label, mode in (("parent", "off"), ("this build", "off"), ("this build", "on")):
            v = [x[key] for x in rows if x["what"] == what and x["label"] == label and x["mode"] == mode]
            if v:
                r[f"{label}, {mode}"] = [min(v), max(v)]
        p, t = r.get("parent, off"), r.get("this build, off")
        if p and t:
            spread = p[1] - p[0]
            r["rule_holds"] = bool(t[0] <= p[1] + spread)          # overlaps, or lies above by at most the parent's spread
            ok = ok and r["rule_holds"]
        out[what] = r
    out["gather_stats"] = [x for x in rows if x["what"] == "gather_stats"]
    print(json.dumps(out, indent=1))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--moves", type=int, default=2)
    ap.add_argument("--edges-per-node", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        raise SystemExit(summarise(a.summarise))
    import torch                                                                # (before any load of the library: one HIP runtime per process)
    from alphazeroforhnefatafl_amd import _lib, abi
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        probe = C.CDLL(_lib.LIB_PATH)                                           # an older build: bind what it exports
        _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
    from alphazeroforhnefatafl_amd._lib import lib
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    if not torch.cuda.is_available():
        raise SystemExit("measure_search_stats: no GPU - nothing is measured without one")
    L = lib()
    has = any(s[0] == "tafl_examples_create_ex" for s in _lib.SYMBOLS)
    if not has:                                                                 # (flags = 0 is exactly tafl_examples_create)
        L.tafl_examples_create_ex = lambda ctx, g, m, k, flags, out: L.tafl_examples_create(ctx, g, m, k, out)
    modes = a.modes.split(",")
    if "on" in modes and not has:
        raise SystemExit("measure_search_stats: this build of the library has no search statistics (--modes off)")
    dev = torch.device("cuda:0")
    G, K, side = a.games, 64, 11
    lg = BatchedGameLogic(abi.rules.COPENHAGEN, side, 128)
    A = lg.action_size
    stream = torch.cuda.ExternalStream(L.tafl_ctx_stream(lg._h))
    torch.manual_seed(0)
    pri = torch.rand((G, A), dtype=torch.float32, device=dev)
    val = torch.zeros(G, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b = lg.new_batch(G, abi.boards.COPENHAGEN)
    done = lg.new_batch(G, abi.boards.COPENHAGEN)
    done.random_advance(5, (C.c_uint32 * G)(*[100000] * G), 0)                 # every game played to its end: what the examples are finalized against

    def emit(row):
        row.update(label=a.label, games=G, sims_per_root=a.sims, moves=a.moves)
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def one_run(ex):
        b.reset_fen(abi.boards.COPENHAGEN, abi.rules.COPENHAGEN.starting_side)
        ex.clear()
        b.gselfplay_begin(ex, a.moves, a.sims, 1.0, a.edges_per_node, game_id_base=0, sample_seed=3, temp_moves=a.moves)
        rounds, w = 1, b.gselfplay_step()
        while w:
            w = b.gselfplay_step(pri.data_ptr(), val.data_ptr(), device=True)
            rounds += 1
        b.gselfplay_end(want_plays=False)
        return rounds

    def timed(call):
        us = []
        for k in range(a.launches + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if k:
                us.append(1e3 * e0.elapsed_time(e1))
        return min(us), max(us)

    exs = {m: lg.new_examples(G, a.moves, K, search_stats=(m == "on")) for m in modes}
    for m in modes:                                                             # untimed: the arena, the code objects
        one_run(exs[m])
    lg.sync(); torch.cuda.synchronize()
    for rep in range(a.reps):
        for m in modes:
            lg.sync(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            rounds = one_run(exs[m])
            lg.sync(); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit({"what": "round", "mode": m, "rep": rep, "seconds": round(dt, 4), "rounds": rounds, "ms_per_round": round(1e3 * dt / rounds, 4),
                  "faults": b.gmcts_stats().faults})
    # (c) the ingest and the gather, on the examples of the last runs
    E = G * a.moves
    for m in modes:
        ex = exs[m]
        ex.finalize(done)
        for rep in range(a.reps):
            pool = lg.new_pool(E, K)
            if m == "on":
                pool.set_search_stats(True)
            lo, hi = timed(lambda: pool.ingest(ex))
            taken = pool.stats().written // (a.launches + 1)
            emit({"what": "ingest", "mode": m, "rep": rep, "ingest_us_min": round(lo, 1), "ingest_us_max": round(hi, 1), "taken": int(taken),
                  "extra_bytes_read": int(8 * K * E) if m == "on" else 0})
            pool.close()
    if "on" in modes:
        ex = exs["on"]
        for rows in (4096, 65536):
            idx = (torch.arange(rows, dtype=torch.int64, device=dev) * 7919 % E).to(torch.int32)
            v, s = torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            vp = C.c_void_p
            lo, hi = timed(lambda: _lib.check(L.tafl_examples_gather_stats(ex._h, vp(idx.data_ptr()), rows, vp(v.data_ptr()), vp(s.data_ptr()), 1)))
            nc = ex.read(idx.cpu().numpy().astype("uint32")[:512])[0]
            mean_children = float(nc.mean())
            emit({"what": "gather_stats", "mode": "on", "rows": rows, "us_min": round(lo, 1), "us_max": round(hi, 1), "mean_stored_children": round(mean_children, 2),
                  "bytes_moved_estimate": int(rows * (4 + 4 + 8 + mean_children * 12 + 8))})
    b.close(); done.close()


if __name__ == "__main__":
    main()
