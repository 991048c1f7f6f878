#!/usr/bin/env python3
"""What the value targets from search values (include/taflhip.h TAFL_EXAMPLES_VALUE_TARGETS) cost on one MI355X, by
the protocol of tools/measure_search_stats.py: 65 536 Copenhagen 11x11 lanes from the start position, S = 64 simulations per root, a
constant-prior evaluator resident in HBM, max_children = 64, an episodes run with a lane budget of `--moves` (32).

round     the library's share of a round: the wall time of one whole run - tafl_gselfplay_begin_episodes, every tafl_gselfplay_step -
          over its rounds.  Mode `off`: an examples object with flags 0, nothing of the feature runs; mode `on`: both flags,
          k_gselfplay_record_stats and k_gselfplay_mark_boundary follow every round.
ingest    tafl_pool_ingest of the run's examples (not finalized: the last episode of every lane is open) between two events on the
          library's stream, one warm-up and `--launches` calls: mode `off` into a pool without settings, mode `on` into a pool with
          search statistics and value targets on, after tafl_examples_value_targets.
targets   (mode `on`) tafl_examples_value_targets(0.9) the same way, with the bytes its two passes move, and `taken` of an ingest into a
          plain pool without and with TAFL_VT_SETTLE_UNFINISHED beside the recorded rows: the share unfinished episodes cost.

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
    out["targets"] = [x for x in rows if x["what"] in ("targets", "taken")]
    print(json.dumps(out, indent=1))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--moves", type=int, default=32)
    ap.add_argument("--edges-per-node", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=3)
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
        raise SystemExit("measure_value_targets: no GPU - nothing is measured without one")
    L = lib()
    modes = a.modes.split(",")
    if "on" in modes and not any(s[0] == "tafl_examples_value_targets" for s in _lib.SYMBOLS):
        raise SystemExit("measure_value_targets: this build of the library has no value targets (--modes off)")
    dev = torch.device("cuda:0")
    G, K, side = a.games, 64, 11
    lg = BatchedGameLogic(abi.rules.COPENHAGEN, side, 128)
    A = lg.action_size
    stream = torch.cuda.ExternalStream(L.tafl_ctx_stream(lg._h))
    pri = torch.ones((G, A), dtype=torch.float32, device=dev)
    val = torch.zeros(G, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b = lg.new_batch(G, abi.boards.COPENHAGEN)

    def emit(row):
        row.update(label=a.label, games=G, sims_per_root=a.sims, lane_budget=a.moves)
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def one_run(ex):
        b.reset_fen(abi.boards.COPENHAGEN, abi.rules.COPENHAGEN.starting_side)
        ex.clear()
        b.gselfplay_begin_episodes(ex, a.moves, a.sims, 1.0, a.edges_per_node, game_id_base=0, sample_seed=3, temp_moves=a.moves)
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

    exs = {m: lg.new_examples(G, a.moves, K, search_stats=(m == "on"), **({"value_targets": True} if m == "on" else {})) for m in modes}
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
    E = G * a.moves
    recorded = {m: int(exs[m].counts()[1]) for m in modes}
    if "on" in modes:                                                           # the targets first: the `on` ingest needs a standing result
        ex = exs["on"]
        plain = lg.new_pool(E, K)
        before = plain.ingest(ex)
        plain.clear()
        lo, hi = timed(lambda: ex.value_targets(0.9))
        res = ex.value_targets(0.9)
        lens = list(ex.counts()[0])
        cols = [j * G + g for g in range(0, G, max(1, G // 64)) for j in range(lens[g])][:4096]
        mean_children = float(ex.read(cols)[0].mean()) if cols else 0.0
        emit({"what": "targets", "mode": "on", "us_min": round(lo, 1), "us_max": round(hi, 1), "recorded": recorded["on"], "episodes_closed": int(res.episodes_closed),
              "episodes_unfinished": int(res.episodes_unfinished), "rows_with_target": int(res.rows_with_target), "mean_stored_children": round(mean_children, 2),
              "bytes_moved_estimate": int(E * 4 + recorded["on"] * (4 + mean_children * 8 + 5) + G * 4 + recorded["on"] * (19 + 5))})
        settled = ex.value_targets(0.9, settle_unfinished=True)
        after = plain.ingest(ex)
        emit({"what": "taken", "mode": "on", "recorded": recorded["on"], "taken_without_settle": int(before[0]), "skipped_open_without_settle": int(before[1]),
              "taken_with_settle": int(after[0]), "skipped_open_with_settle": int(after[1]), "rows_settled": int(settled.rows_settled),
              "share_lost_without_settle": round(1.0 - before[0] / max(1, recorded["on"]), 4)})
        plain.close()
    for m in modes:
        ex = exs[m]
        for rep in range(a.reps):
            pool = lg.new_pool(E, K)
            if m == "on":
                pool.set_search_stats(True)
                pool.set_value_targets(True)
            lo, hi = timed(lambda: pool.ingest(ex))
            taken = pool.stats().written // (a.launches + 1)
            emit({"what": "ingest", "mode": m, "rep": rep, "ingest_us_min": round(lo, 1), "ingest_us_max": round(hi, 1), "taken": int(taken), "recorded": recorded[m],
                  "extra_bytes_moved": int(taken * 10 + E * 9) if m == "on" else 0})
            pool.close()
    b.close()


if __name__ == "__main__":
    main()
