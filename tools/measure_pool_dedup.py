"""De-duplication of the training pool (tafl_pool_dedup / _gather_dedup / _weights_from_dedup): what the new calls
cost beside a tafl_pool_ingest, and how redundant the rows of self-play runs from the start position are.

The pool: capacity 4 Mi rows, filled by the ingests of `--runs` rollout-mode tafl_selfplay_record runs of `--games` Copenhagen 11x11
lanes from the start position x up to `--moves` moves each (S = --sims, the first --temp-moves plays drawn from the visit counts;
every run has its own seeds and game ids), every example counted as finished.  Each recorded row is ingested ONCE; a game that ends
before `--moves` leaves fewer rows, and the ring drops the oldest rows beyond its capacity.  µs per call from HIP events on the
context's stream, one warm-up, `--launches` timed calls, min..max:
  * tafl_pool_ingest of the last run's rows into a second pool of exactly that many slots (every timed call stores the same rows);
    the scale is given per row;
  * tafl_pool_dedup without and with TAFL_POOL_DEDUP_SYMMETRIES (three kernels, two memsets, a 32-byte read-back), and what it found:
    distinct / live, largest, collisions;
  * tafl_pool_weights_from_dedup; tafl_pool_gather_dedup of 4 096 rows with device pointers.
--parent-calls times tafl_pool_ingest and tafl_pool_sample_weighted at 4 096 rows alone (one run) and takes --lib, so that this commit
and its parent's build can take turns.  Builds with -DTAFL_POOLDD_AGGREGATE=0 (every lane of k_pooldd_insert inserts its own row) and =2
(a loop over the wave's distinct keys) are compared by --lib as well.  --label names the build in the output.  Time per kernel:
the same command under `rocprofv3 --kernel-trace --stats`, in a run of its own.

    python tools/measure_pool_dedup.py [--launches 3] [--json out.json] [--parent-calls] [--lib path/to/libtaflhip.so] [--label name]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alphazeroforhnefatafl_amd import _lib, abi  # noqa: E402


def timed(stream, launches, torch, call):
    us = []
    for k in range(launches + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if k:
            us.append(1e3 * e0.elapsed_time(e1))
    return [min(us), max(us)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--moves", type=int, default=64)
    ap.add_argument("--sims", type=int, default=8)
    ap.add_argument("--cap", type=int, default=32)
    ap.add_argument("--temp-moves", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--label", default=None)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--parent-calls", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch                                                                # (before any load of the library: one HIP runtime per process)
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        if a.parent_calls:                                                      # an older build: bind what it exports
            probe = C.CDLL(_lib.LIB_PATH)
            _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
    from alphazeroforhnefatafl_amd._lib import check, lib
    from alphazeroforhnefatafl_amd.abi import TaflPoolIngestResult
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    G, moves, K = a.games, a.moves, 16
    lg = BatchedGameLogic(abi.rules.COPENHAGEN, 11, 128)
    n, A = lg.side_len, lg.action_size
    stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
    vp = C.c_void_p
    dev = torch.device("cuda", 0)
    runs = 1 if a.parent_calls else a.runs
    Cp = G * moves if a.parent_calls else a.capacity
    pool = lg.new_pool(Cp, K)
    ex = lg.new_examples(G, moves, K)
    done = lg.new_batch(G, abi.boards.COPENHAGEN)
    done.random_advance(5, (C.c_uint32 * G)(*[100000] * G), 0)               # every game played to its end
    taken = []
    for r in range(runs):                                                       # every recorded row is ingested once
        ex.clear()
        b = lg.new_batch(G, abi.boards.COPENHAGEN)
        b.selfplay_record(ex, moves, a.sims, 1.0, 2 + r, a.cap, game_id_base=r * G, sample_seed=11 + r, temp_moves=a.temp_moves, want_plays=False)
        ex.finalize(done)
        b.close()
        taken.append(int(pool.ingest(ex)[0]))
    done.close()
    res = {"games": G, "moves": moves, "runs": runs, "sims": a.sims, "temp_moves": a.temp_moves, "max_children": K, "build": a.label or _lib.LIB_PATH,
           "launches": a.launches, "capacity": Cp, "taken_per_run": taken, "live": int(pool.stats().live)}
    out = TaflPoolIngestResult()
    tpool = lg.new_pool(taken[-1], K)                                           # exactly the last run's rows: every timed ingest stores the same rows
    res["ingest_us"] = timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_ingest(tpool._h, ex._h, C.byref(out))))
    res["ingest_rows"] = int(out.taken)
    assert int(tpool.stats().live) == taken[-1] == int(out.taken)
    tpool.close()
    pool.set_weighting(1)
    rows = 4096
    o = dict(boards=torch.empty((rows, n, n), dtype=torch.uint8, device=dev), sides=torch.empty(rows, dtype=torch.uint8, device=dev),
             pi=torch.empty((rows, A), dtype=torch.float32, device=dev), z=torch.empty(rows, dtype=torch.float32, device=dev),
             slot=torch.empty(rows, dtype=torch.int32, device=dev), sym=torch.empty(rows, dtype=torch.uint8, device=dev),
             weight=torch.empty(rows, dtype=torch.int32, device=dev), total=torch.zeros(1, dtype=torch.int64, device=dev))
    step = [0]

    def weighted():
        step[0] += 1
        check(lib().tafl_pool_sample_weighted(pool._h, 7, step[0], 0, rows, abi.POOL_SAMPLE_SYM, vp(o["boards"].data_ptr()), vp(o["sides"].data_ptr()), vp(o["pi"].data_ptr()),
                                              vp(o["z"].data_ptr()), vp(o["slot"].data_ptr()), vp(o["sym"].data_ptr()), vp(o["weight"].data_ptr()), vp(o["total"].data_ptr()), 1))

    pool.weight_stats()                                                         # the rebuild is done
    torch.cuda.synchronize()
    res["sample_weighted_4096_us"] = timed(stream, a.launches, torch, weighted)
    if not a.parent_calls:
        from alphazeroforhnefatafl_amd.abi import TaflPoolDedupCfg, TaflPoolDedupResult, TaflPoolDedupWeights
        for symmetries in (0, 1):
            cfg, r = TaflPoolDedupCfg(flags=symmetries, key_bits=64), TaflPoolDedupResult()
            us = timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_dedup(pool._h, C.byref(cfg), C.byref(r))))
            res["dedup_symmetries_us" if symmetries else "dedup_us"] = us
            res["found_symmetries" if symmetries else "found"] = dict(live=int(r.live), distinct=int(r.distinct), distinct_per_live=r.distinct / r.live, largest=int(r.largest),
                                                                      collisions=int(r.collisions), device_bytes=int(r.device_bytes))
        w = TaflPoolDedupWeights(scale=1 << 20, flags=0)
        res["weights_from_dedup_us"] = timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_weights_from_dedup(pool._h, C.byref(w))))
        sl = torch.from_numpy(np.random.default_rng(1).integers(0, Cp, rows).astype(np.int32)).to(dev)
        rep, mult, zm = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        res["gather_dedup_4096_us"] = timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_gather_dedup(pool._h, vp(sl.data_ptr()), rows, vp(rep.data_ptr()),
                                                                                                                  vp(mult.data_ptr()), vp(zm.data_ptr()), 1)))
        res["sample_weighted_4096_after_dedup_weights_us"] = timed(stream, a.launches, torch, weighted)
        res["pool_device_bytes"] = int(pool.stats().device_bytes)
    pool.close()
    for k, v in res.items():
        print(k, json.dumps(v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
